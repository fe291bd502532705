"""The Laplace and Color cases that must equal the CPU oracle BIT FOR BIT in the exact flavour (lvm_debug_exact_lab: OpenCV's
operation order, no transcendental function on the way) -- one matrix, run on the CPU emulation build by tests/test_emu_parity.py
and on the gfx950 build by tests/test_gpu_exact.py.  Each body takes the library behind the C ABI (`lib`) and, where it passes
device pointers, a memory adaptor (helpers.HostMem / helpers.TorchMem).  Lists hold Riesz entries where the emulation test of the
same name covers all three modes; the GPU module keeps the Laplace and Color ones (Riesz calls acosf / sinf / cosf, see
tests/test_gpu_exact.py)."""
import os
import re

import numpy as np

import content
from helpers import far_clip, far_units, frames_clip, layout_clip, run_pair


def _color_fps(ck, pk, fps=15.0):
    ck["fps"] = fps
    pk["framerate"] = fps


def _clip(lvm, ck, kind=None):
    """the synthetic clip, or the chromatic content `kind` of tests/content.py in its place"""
    return lvm.synth.Clip(**ck) if kind is None else content.chroma_clip(lvm, ck, kind)


# ---- Laplace ---------------------------------------------------------------------------------------
LAPLACE_SHAPES = [(160, 90, 3, 3), (135, 77, 4, 3), (100, 64, 2, 1), (64, 48, 1, 3), (67, 131, 3, 3), (40, 23, 2, 3), (320, 180, 4, 3),
                  (404, 300, 5, 3), (330, 200, 6, 3)]


def laplace_shape(lvm, po, lib, w, h, levels, ch):
    ck, pk = lvm.synth.config(0, (w, h, levels))
    ck["channels"] = ch
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 6, 0.0, exact=True)


ANALYTIC = [(0, 135, 77, 4), (0, 328, 109, 3), (2, 135, 77, 3), (2, 264, 150, 3)]


def analytic_flavour(lvm, po, lib, monkeypatch, idx, w, h, levels, kind=None, exact=True):
    """lvm_debug_lab_analytic: the cube-root forward Lab (OpenCV with its interpolation switched off) in the kernels that
    convert from the u8 frame themselves, against the oracle with lvmo_set_lab_lut(0); scalar and 4-pixel variants, strip
    first kernel forced on."""
    monkeypatch.setenv("LVM_D0_MIN_TASKS", "0")
    ck, pk = lvm.synth.config(idx, (w, h, levels))
    return run_pair(lvm, po, lib, _clip(lvm, ck, kind), pk, 5, 0.0 if exact else 1e-4, exact=exact, analytic=True)


def laplace_param_changes_and_reset(lvm, po, lib):
    ck, pk = lvm.synth.config(0, (96, 64, 3))

    def vary(t, p):
        if t >= 3:
            p["amplification"] = 35.0
            p["coLow"] = 0.0            # exercises the lo == 0 -> 0.01 rule (TemporalFilter.cpp:11-12)
        if t >= 5:
            p["levels"] = 2             # structural change -> state reset
        return p
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 8, 0.0, exact=True, param_fn=vary)


PIPELINED = [(160, 90, 3), (320, 180, 4), (135, 77, 4), (64, 48, 1)]

FUSED_MULTI = [(1000, 760, 6), (800, 600, 4), (1001, 763, 5)]


def laplace_shape_3_frames(lvm, po, lib, w, h, levels):
    ck, pk = lvm.synth.config(0, (w, h, levels))
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 3, 0.0, exact=True)


FIN_ROWS = [4, 8, 16]


def laplace_final_strip_height(lvm, po, lib, monkeypatch, rows, kind=None):
    """k_lap_final_v4 walks strips of `rows` output rows per wave (the launch code shortens them for small frames): force the
    long strips, on a height that leaves a partial last strip and a width with a partly filled last wave."""
    monkeypatch.setenv("LVM_FIN_ROWS", str(rows))
    monkeypatch.setenv("LVM_FIN_MIN_TASKS", "0")
    ck, pk = lvm.synth.config(0, (328, 90 + 2 * rows + 3, 3))
    return run_pair(lvm, po, lib, _clip(lvm, ck, kind), pk, 4, 0.0, exact=True)


ROWS_PYRDOWN = [(328, 109, 3), (1000, 760, 5), (520, 77, 4)]


def laplace_wave_strip_pyrdown(lvm, po, lib, monkeypatch, w, h, levels):
    """k_pyr_down_rows (the pyrDown of large planes) forced onto every level whose width allows it."""
    monkeypatch.setenv("LVM_ROWS_MIN_ELEMS", "0")
    return laplace_shape_3_frames(lvm, po, lib, w, h, levels)


FIRST_KERNEL = [(0, 328, 109, 3), (0, 1000, 70, 4), (0, 124 * 2 * 2, 40, 2), (3, 264, 90, 3), (3, 96, 77, 2)]


def wave_strip_first_kernel(lvm, po, lib, monkeypatch, idx, w, h, levels):
    """k_down0_rows (u8 -> Lab / float -> pyrDown with DPP halo exchange between lanes) forced onto small frames."""
    monkeypatch.setenv("LVM_D0_MIN_TASKS", "0")
    ck, pk = lvm.synth.config(idx, (w, h, levels))
    if idx == 3:
        _color_fps(ck, pk)
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 4, 0.0, exact=True)


FUSED_TABLE = [(328, 109, 3, True), (1000, 70, 4, True), (124 * 2 * 2, 40, 2, True), (264, 90, 3, False)]


def fused_table_first_kernel(lvm, po, lib, monkeypatch, w, h, levels, exact):
    """k_down0_lut_rows (OpenCV's forward Lab table + pyrDown + the integer planes of the owned pixels in one pass) forced onto
    small frames.  exact=False: the default flavour's fma tap sums against the 1e-4 bar."""
    monkeypatch.setenv("LVM_D0_FUSED_WAVES", "1")
    ck, pk = lvm.synth.config(0, (w, h, levels))
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 4, 0.0 if exact else 1e-4, exact=exact)


def unfused_conversion_in_batches(lvm, po, lib, mem, monkeypatch):
    """LVM_D0_FUSED=0: labconv.hip's conversion kernel + the plane-reading first kernels in temporal batches."""
    monkeypatch.setenv("LVM_D0_FUSED", "0")
    frames_clip(lvm, po, lib, mem, 0, 320, 180, 4, 1, (1, 6, 5))


LEVEL1_GEOMETRIES = [
    (320, 180, 2, 1, (1, 4, 3)),        # two levels: level 1 is the top live level (no cur_2), too large for the tail kernel
    (264, 74, 3, 1, (1, 6, 1, 2)),      # partial tiles right and below, per-frame calls in between
    (132, 70, 3, 2, (1, 5, 3)),         # level 2 with an odd width: level chain for level 2; two streams
    (160, 91, 3, 1, (1, 4, 4)),         # odd frame height (pyrUp with dsize = 2 n - 1 on both steps)
    (520, 150, 4, 1, (1, 9)),           # five tiles across: interior tiles without any border lane
    (128, 16, 2, 1, (1, 3, 3)),         # exactly one tile
]


def laplace_param_change_between_calls(lvm, po, lib):
    """amplification / chromAttenuation change between calls: the level-1 states carry over, frames keep matching the oracle"""
    ck, pk = lvm.synth.config(0, (264, 74, 3))

    def vary(t, q):
        if t >= 5:
            q["amplification"] = 35.0; q["chromAttenuation"] = 0.4
        return q
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 9, 0.0, exact=True, param_fn=vary)


def fused_conversion_two_streams(lvm, po, lib, mem, monkeypatch):
    monkeypatch.setenv("LVM_D0_FUSED_WAVES", "1")
    frames_clip(lvm, po, lib, mem, 0, 264, 90, 3, 2, (1, 5, 4))


LAPLACE_BATCHES = [(160, 90, 3, 1, (1, 4, 3, 1, 5)), (320, 180, 4, 1, (5, 6)), (135, 77, 4, 2, (3, 3, 2)), (404, 300, 5, 1, (2, 7)),
                   (64, 48, 1, 1, (3, 3)), (200, 120, 4, 1, (1, 11, 17, 9))]   # deeper than the prefetch ring of k_lap_up

SPLIT_LEVELS = [(640, 360, 5, 1, (1, 8, 4)), (256, 256, 6, 1, (1, 4, 6)), (320, 182, 5, 2, (1, 5, 16)), (576, 72, 4, 1, (1, 4, 4)),
                (512, 384, 7, 1, (1, 4))]   # 7 levels: five decoupled levels, the top one 8 x 6

SPLIT_FROM_2 = SPLIT_LEVELS[:3]


def laplace_split_from_2(lvm, po, lib, mem, monkeypatch, w, h, levels, ns, calls):
    """LVM_LAP_SPLIT_FROM=2: levels 2 .. L-1 all in the IIR + collapse launches."""
    monkeypatch.setenv("LVM_LAP_SPLIT_FROM", "2")
    frames_clip(lvm, po, lib, mem, 0, w, h, levels, ns, calls)


def laplace_level_chain(lvm, po, lib, mem, monkeypatch):
    """LVM_LAP_SPLIT=0 keeps the level-by-level chain of fused launches in temporal batches."""
    monkeypatch.setenv("LVM_LAP_SPLIT", "0")
    frames_clip(lvm, po, lib, mem, 0, 320, 180, 4, 1, (1, 8, 4))


BLOCK_UP = [(328, 109, 3, (1, 4, 8, 2, 3)), (200, 120, 4, (1, 16, 6))]


def laplace_tiled_up(lvm, po, lib, mem, monkeypatch):
    """LVM_UP_ROWS=0 selects the LDS-tiled k_lap_up (the kernel odd-width levels always use)."""
    monkeypatch.setenv("LVM_UP_ROWS", "0")
    frames_clip(lvm, po, lib, mem, 0, 200, 120, 4, 1, (1, 8, 5))


# ---- Colour ----------------------------------------------------------------------------------------
# (at least 12 frames per clip: with a window of a few columns the ideal band-pass passes nothing, the magnified signal is zero
# and neither the pyramid nor the up-chain arithmetic would influence the output -- checked by mutating the kernels)
COLOR_SHAPES = [(96, 64, 3, 3, 60.0), (135, 77, 4, 3, 30.0), (64, 48, 1, 3, 7.0), (67, 131, 2, 1, 15.0)]


def color_shape(lvm, po, lib, w, h, levels, ch, fps):
    ck, pk = lvm.synth.config(3, (w, h, levels))
    ck["channels"] = ch
    _color_fps(ck, pk, fps)
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 20, 0.0, exact=True)


def color_12_frames(lvm, po, lib, monkeypatch, w, h, levels, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ck, pk = lvm.synth.config(3, (w, h, levels))
    _color_fps(ck, pk)
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 12, 0.0, exact=True)


COL_OUT_ROWS = [(264, 90, 3, "0"), (264, 90, 3, "2"), (264, 90, 3, "8"), (264, 90, 3, "36"), (96, 77, 2, "16")]
COL_STRIP_BORDERS = [(516, 40, 2), (772, 24, 2), (256, 64, 3)]
COL_PREVIOUS_STRIPS = [(264, 90, 3), (512, 128, 4)]
COL_DOWN01_ROWS = [(264, 90, 3, "7"), (264, 90, 3, "17"), (96, 77, 2, "1"), (96, 77, 2, "4"), (520, 52, 3, "7"), (128, 37, 3, "17"),
                   (512, 128, 4, "4")]


def color_wide_band_and_fps_change(lvm, po, lib):
    ck, pk = lvm.synth.config(3, (64, 48, 2))
    pk["coLow"] = 0.0; pk["coHigh"] = 40.0                   # every packed element passes (lo == 0 -> 0.01)

    def vary(t, p):
        if t >= 12:
            p["framerate"] = 7.0                              # window cap shrinks 128 -> 16: one column dropped per frame
        return p
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 24, 0.0, exact=True, param_fn=vary)


COLOR_BATCHES = [(64, 48, 2, 1, (18, 5, 7, 3)), (40, 30, 1, 2, (20, 6)), (80, 52, 3, 1, (17, 16, 9)),
                 (48, 32, 2, 1, (18, 40, 35))]   # calls longer than one batch (32 frames) are cut
COLOR_BATCH_PARAMS = ({"framerate": 7.0, "coLow": 0.4, "coHigh": 2.0}, {"fps": 7.0})

NARROW_DFT_BANDS = [(0.8, 1.6), (2.9, 3.5), (0.8, 0.95)]


def color_narrow_band_dft(lvm, po, lib, mem, monkeypatch, lo, hi, thin8):
    monkeypatch.setenv("LVM_COL_THIN8_DFT", thin8)
    frames_clip(lvm, po, lib, mem, 3, 64, 48, 2, 1, (18, 5, 7, 9), over={"framerate": 7.0, "coLow": lo, "coHigh": hi},
                clip_over={"fps": 7.0})


# ---- Riesz (phase) ---------------------------------------------------------------------------------
# Run on the CPU emulation build by tests/test_emu_parity.py (host libm on both sides) and on the gfx950 build by
# tests/test_gpu_riesz_exact.py under portable_trig() below: csrc/rz_trig.h on both sides, so the GPU owes the oracle's bits too.
def portable_trig(monkeypatch, po, oracle_bits=()):
    """LVM_RZ_PORTABLE_TRIG=1 for the contexts created from here on (monkeypatch restores it) and LVMO_VAR_PORTABLE_TRIG, plus
    `oracle_bits` (names of po.VARIANTS), for the oracle: the caller -- a fixture -- sets the oracle's mask back to 0 when the test ends"""
    monkeypatch.setenv("LVM_RZ_PORTABLE_TRIG", "1")
    mask = po.VARIANTS["portable_trig"] | sum(po.VARIANTS[b] for b in oracle_bits)
    po.set_variant(mask)
    return mask


PTRIG_NAMES = ("rz_phase", "rz_phase_small", "rz_blur_amp", "rz_blur_amp_small", "rz_blur_amp_tiles")


def ptrig_launches(names):
    """of {report name: variants}: the phase and blur / amplify launches, each of which must have run as a `ptrig` variant and nothing else"""
    got = {n: v for n, v in names.items() if n in PTRIG_NAMES}
    assert any(n.startswith("rz_phase") for n in got) and any(n.startswith("rz_blur_amp") for n in got), names
    for n, v in got.items():
        assert v and all("ptrig" in x.split("+") for x in v), (n, v)
    return got


def no_ptrig_launches(names):
    assert not any("ptrig" in x for v in names.values() for x in v), names


def profiled_call(lvm, lib, mem, w, h, levels, env=None, kind=0, nframes=3, exact_lab=True):
    """one profiled lvm_process_device_frames call of `nframes` frames behind two seeding per-frame calls, exact flavour:
    ({report name: variants} of that call, its output frames, its input frames)"""
    import os
    ck, pk = lvm.synth.config(2, (w, h, levels))
    clip = lvm.synth.Clip(**ck)
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    ctx = None
    fb = w * h * 3
    try:
        ctx = lvm.Context(0, 1, lib)
        ctx.exact_lab(exact_lab)
        if kind:
            ctx.set_opencv_build(kind)
        cp = lvm.LvmParams(pk["mode"], pk["levels"], pk["amplification"], pk["coWavelength"], pk["coLow"], pk["coHigh"], pk["chromAttenuation"],
                           pk["framerate"], 0)
        fin = np.stack([clip.frame(t) for t in range(2 + nframes)])
        d_in = mem.upload(fin)
        d_out = mem.zeros_like(d_in)
        for t in range(2):
            ctx.process_device_frames(cp, 1, mem.ptr(d_in, t), w, h, 3, w * 3, fb, fb, mem.ptr(d_out, t), w * 3, fb, fb, mem.stream())
        mem.sync(ctx)
        ctx.profile(True)
        prod = ctx.process_device_frames(cp, nframes, mem.ptr(d_in, 2), w, h, 3, w * 3, fb, fb, mem.ptr(d_out, 2), w * 3, fb, fb, mem.stream())
        mem.sync(ctx)
        assert all(prod), prod
        variants = ctx.profile_variants()
        names = {n: variants.get(n, set()) for n in ctx.profile_collect()}
        return names, np.array(mem.download(d_out), copy=True), fin
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if ctx is not None:
            ctx.close()


RIESZ_SHAPES = [(96, 64, 3), (135, 77, 4), (64, 48, 1), (67, 131, 2), (160, 90, 5), (134, 78, 2)]


def riesz_shape(lvm, po, lib, w, h, levels):
    ck, pk = lvm.synth.config(2, (w, h, levels))
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 6, 0.0, exact=True)


RIESZ_TILE_KERNELS = [(264, 150, 3, (2, 1, 2)), (160, 90, 5, (2, 3)), (96, 64, 3, (2, 1, 1))]


def riesz_wide_and_narrow_tile_kernels(lvm, po, lib, mem, monkeypatch, w, h, levels, calls, wide):
    """k_rz_split2 / k_rz_phase4 (wide = "1") or k_rz_split / k_rz_phase ("0") forced onto small frames, per-frame calls between
    temporal batches"""
    monkeypatch.setenv("LVM_RZ_SPLIT2_MIN", "0" if wide == "1" else "1000000000")
    monkeypatch.setenv("LVM_RZ_PHASE4_MIN_FRAMES", "1" if wide == "1" else "2")
    monkeypatch.setenv("LVM_RZ_SPLIT_ROWS", "0")
    frames_clip(lvm, po, lib, mem, 2, w, h, levels, 1, calls)


def riesz_register_blocked_blur(lvm, po, lib, monkeypatch, blur4):
    monkeypatch.setenv("LVM_RZ_BLUR4", blur4)
    monkeypatch.setenv("LVM_RZ_BLUR_STRIPS", "0")         # (the strip form is the default for every even-width level since round 5)
    ck, pk = lvm.synth.config(2, (264, 150, 3))
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 4, 0.0, exact=True)


RIESZ_STRIP_BLUR = [(264, 150, 3, "16", True), (134, 78, 2, "64", True), (520, 70, 3, "32", True), (264, 150, 3, "16", False)]


def riesz_strip_blur(lvm, po, lib, monkeypatch, w, h, levels, rows, exact):
    monkeypatch.setenv("LVM_RZ_BLUR_STRIPS_MIN", "0")
    monkeypatch.setenv("LVM_RZ_BLUR_STRIP_ROWS", rows)
    ck, pk = lvm.synth.config(2, (w, h, levels))
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 4, 0.0 if exact else 1e-4, exact=exact)


def riesz_strip_blur_in_temporal_batches(lvm, po, lib, mem, monkeypatch):
    monkeypatch.setenv("LVM_RZ_BLUR_STRIPS_MIN", "0")
    monkeypatch.setenv("LVM_RZ_BLUR_STRIP_ROWS", "32")
    frames_clip(lvm, po, lib, mem, 2, 264, 150, 3, 2, (2, 4, 1))


def riesz_tiled_blur(lvm, po, lib, monkeypatch):
    monkeypatch.setenv("LVM_RZ_BLUR_STRIPS", "0")
    ck, pk = lvm.synth.config(2, (264, 150, 3))
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 3, 0.0, exact=True)


def riesz_collapse_tile_variants(lvm, po, lib, monkeypatch, compact):
    monkeypatch.setenv("LVM_RZ_COMPACT", compact)
    ck, pk = lvm.synth.config(2, (264, 150, 3))
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 3, 0.0, exact=True)


def riesz_cutoff_change_gray_and_reset(lvm, po, lib):
    ck, pk = lvm.synth.config(2, (96, 64, 3))

    def vary(t, p):
        if t >= 3:
            p["coLow"] = 1.0            # MagnifyCore.hpp:243-248: new coefficients, filters cleared, prior rebuilt
        if t >= 5:
            p["coHigh"] = 5.0
        if t >= 7:
            p["levels"] = 2             # structural change: re-init => passthrough frame
        return p
    run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 10, 0.0, exact=True, param_fn=vary)
    gray = lvm.synth.Clip(96, 64, channels=1)
    run_pair(lvm, po, lib, gray, pk, 3, 0.0, exact=True)    # < 3 channels: always passthrough (:212)


RIESZ_BATCHES = [(96, 64, 3, 1, (2, 5, 3)), (135, 77, 4, 2, (3, 4)), (160, 90, 5, 1, (6, 2)), (64, 48, 1, 1, (4,))]
RIESZ_SPLIT_STRIPS = (["0", "10", "54"], [(520, 70, 3), (256, 41, 2), (1000, 24, 2), (128, 5, 2)])            # (strip heights, sizes)
RIESZ_COLLAPSE_STRIPS = (["0", "10", "64"], [(512, 64, 4), (520, 70, 2), (1000, 24, 2), (8, 4, 2)])


def riesz_wave_strip_stencils(lvm, po, lib, monkeypatch, w, h, levels, strip):
    monkeypatch.setenv("LVM_RZ_SPLIT_ROWS_MIN", "1")
    monkeypatch.setenv("LVM_RZ_SPLIT_STRIP", strip)
    ck, pk = lvm.synth.config(2, (w, h, levels))
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 4, 0.0, exact=True)


def riesz_wave_strip_collapse_and_output(lvm, po, lib, monkeypatch, w, h, levels, strip):
    monkeypatch.setenv("LVM_RZ_COLLAPSE_STRIPS_MIN", "1")
    monkeypatch.setenv("LVM_RZ_COLLAPSE_STRIP", strip)
    ck, pk = lvm.synth.config(2, (w, h, levels))
    return run_pair(lvm, po, lib, lvm.synth.Clip(**ck), pk, 4, 0.0, exact=True)


# ---- every mode: layouts, degenerate content, parameters, shapes ----------------------------------------------------------
PADDED_STRIDES =[(0, 4, 8), (0, 1, 3), (2, 4, 4), (2, 7, 1), (3, 8, 4), (3, 5, 5)]


# Views into larger buffers (helpers.layout_clip): (extra canvas columns, rx, ry, ox, oy, stream gap bytes, order).  The launch code
# picks the vector kernels where w % 4 == 0 and row strides, stream strides AND both base pointers are multiples of 4, each term
# on its own for the input and for the output; the wave-strip kernels of the production sizes size their buffer resources from the
# row stride.  Row bytes for w = 64: 225 (A), 228 (B, C, D, G).
LAYOUTS = {
    "A": (11, 5, 3, 2, 1, 7, "fs"),             # odd view: rows, streams and both pointers unaligned -> byte kernels in batches
    "B": (12, 4, 2, 8, 1, 4096, "fs"),          # aligned view: vector kernels with stride != w * 3, streams far apart
    "C": (12, 1, 2, 8, 1, 4096, "fs"),          # odd input base only: strides are multiples of 4, the pointer term alone is false
    "D": (12, 4, 2, 3, 1, 4096, "fs"),          # mixed: input vector-eligible, output not (its mirror image is C)
    "E": (0, 0, 0, 0, 0, 6, "fs"),              # packed rows, stream stride h * w * 3 + 6: stream 1 unaligned, stream 0 not (two streams)
    "F": (0, 0, 0, 0, 0, 0, "mosaic"),          # two streams side by side in one frame: stream stride w * 3 < a frame; frame by frame
    "F_device": (0, 0, 0, 0, 0, 0, "mosaic_device"),      # the same through lvm_process_device
    "G": (12, 4, 2, 8, 1, 0, "sf"),             # [stream][frame] order: the batch test of lvm_process_device_frames fails -> frame by frame
}
# per mode: call lengths, parameter overrides, clip overrides (Color: the band of COLOR_BATCH_PARAMS, 18 frames fill its window)
LAYOUT_MODES = {0: ((1, 4, 3), None, None), 2: ((1, 4, 3), None, None),
                3: ((18, 5, 7), {"framerate": 7.0, "coLow": 0.4, "coHigh": 2.0}, {"fps": 7.0})}
LAYOUT_SHAPES = {0: [(64, 48, 3), (61, 45, 3)], 3: [(64, 48, 2), (61, 45, 2)], 2: [(134, 78, 2), (67, 131, 2)]}


def _layout_streams(name):
    return (2,) if name in ("E", "F", "F_device") else (1, 2)


# (mode, w, h, levels, streams, layout) at the default switches: the smallest shapes of the matrix, one with w % 4 == 0 where the mode
# has vector kernels at that size, one odd
LAYOUT_CASES = [(idx, w, h, lv, ns, name) for idx in (0, 3, 2) for (w, h, lv) in LAYOUT_SHAPES[idx] for name in LAYOUTS for ns in _layout_streams(name)]

# the production-size strip kernels forced onto small frames (switches as in FIRST_KERNEL / FUSED_TABLE / FIN_ROWS / ROWS_PYRDOWN /
# COL_DOWN01_ROWS / COL_OUT_ROWS and the Riesz strip tests) on the views that keep them (B), break the input side through the pointer
# term alone (C) and break the output side alone (D); LAYOUT_LAUNCHES says which kernels each mode must then pick
LAYOUT_FORCED = {
    "lap_rows": (0, 328, 109, 3, {"LVM_D0_MIN_TASKS": "0", "LVM_FIN_ROWS": "8", "LVM_FIN_MIN_TASKS": "0", "LVM_ROWS_MIN_ELEMS": "0"}),
    "lap_fused": (0, 328, 109, 3, {"LVM_D0_FUSED_WAVES": "1", "LVM_FIN_ROWS": "8", "LVM_FIN_MIN_TASKS": "0"}),
    "col_down01": (3, 264, 90, 3, {"LVM_D0_MIN_TASKS": "0", "LVM_COL_DOWN01_ROWS": "7", "LVM_COL_OUT_MIN_TASKS": "0"}),
    "col_out_rows": (3, 264, 90, 3, {"LVM_COL_OUT_LEAN": "0", "LVM_COL_OUT_MIN_TASKS": "0"}),
    "rz_strips": (2, 264, 150, 3, {"LVM_RZ_SPLIT_ROWS_MIN": "1", "LVM_RZ_BLUR_STRIPS_MIN": "0", "LVM_RZ_COLLAPSE_STRIPS_MIN": "1",
                                   "LVM_RZ_PHASE4_MIN_FRAMES": "1"}),
}
LAYOUT_FORCED_CASES = [(force, name) for force in LAYOUT_FORCED for name in ("B", "C", "D")]
# What the launch code must pick per forced case and layout: report names (lvm_profile_collect) with the kernel variant that ran under
# them where several kernels share a name (lvm_profile_variants: "strips" = wave strips, "vec4" = tiled with dword-wide frame I/O,
# "bytes" = tiled with byte I/O); None = the name must not be launched.  Read off the launch code, side by side:
#   input side only (w % 4, in strides, d_in):   lab_lut (labconv.hip), col_down0 / col_down01 (col_down)
#   output side only (out strides, d_out):       the Riesz strip output kernel (rz_collapse_out: out_ok) -- so C KEEPS it and D loses it
#   both sides:                                  lap_down0, lap_down0_lut, lap_final (lap_vec4), col_out / col_minmax (col_up_out), tiled rz_final
# so B keeps every strip kernel, C (odd input pointer) and D (odd output pointer) lose exactly the ones whose side they break.
# The last entries of a case are kernels that read float planes only: launched in every layout, they show that the switches reached the state.
_S, _V, _B = {"strips"}, {"vec4"}, {"bytes"}
LAYOUT_LAUNCHES = {
    "lap_rows": {"B": {"lab_lut": _V, "lap_down0": _S, "lap_final": _S}, "C": {"lab_lut": _B, "lap_down0": _B, "lap_final": _B},
                 "D": {"lab_lut": _V, "lap_down0": _B, "lap_final": _B}, "*": {"pyr_down_rows_l1": set()}},      # (batched calls may take lap_down0_lut besides: its threshold counts the CUs)
    "lap_fused": {"B": {"lap_down0_lut": set(), "lab_lut": None, "lap_down0": None, "lap_final": _S},
                  "C": {"lap_down0_lut": None, "lab_lut": _B, "lap_down0": _B, "lap_final": _B},
                  "D": {"lap_down0_lut": None, "lab_lut": _V, "lap_down0": _B, "lap_final": _B}, "*": {}},
    "col_down01": {"B": {"col_down01": set(), "col_down0": None, "col_minmax_u2": set(), "col_out_u2": set(), "col_out": None},
                   "C": {"col_down01": None, "col_down0": _B, "col_minmax_u2": None, "col_out_u2": None, "col_minmax": _B, "col_out": _B},
                   "D": {"col_down01": set(), "col_down0": None, "col_minmax_u2": None, "col_out_u2": None, "col_minmax": _B, "col_out": _B}, "*": {}},
    "col_out_rows": {"B": {"col_down0": _V, "col_minmax": _S, "col_out": _S}, "C": {"col_down0": _B, "col_minmax": _B, "col_out": _B},
                     "D": {"col_down0": _V, "col_minmax": _B, "col_out": _B}, "*": {"col_out_u2": None, "col_down01": None}},
    "rz_strips": {"B": {"lab_lut": _V, "rz_final": _S}, "C": {"lab_lut": _B, "rz_final": _S}, "D": {"lab_lut": _V, "rz_final": _B},
                  "*": {"rz_phase": set(), "rz_phase_small": None, "rz_blur_amp": set(), "rz_blur_amp_small": None, "rz_blur_amp_tiles": None}},
}


def layout_case(lvm, po, lib, mem, idx, w, h, levels, n_streams, name, env=None, exact=True, profile=False, clip_fn=None):
    calls, over, clip_over = LAYOUT_MODES[idx]
    return layout_clip(lvm, po, lib, mem, idx, w, h, levels, n_streams, calls, LAYOUTS[name], env=env, over=over, clip_over=clip_over,
                       exact=exact, profile=profile, clip_fn=clip_fn)


def layout_forced_case(lvm, po, lib, mem, force, name, exact=True, clip_fn=None, ptrig=False, n_streams=1, calls=None, env_extra=None, size=None):
    """one forced case: the bytes, and the kernels LAYOUT_LAUNCHES names for this layout -- a silent fall-back to another kernel family fails.
    ptrig (under portable_trig()): the phase and blur / amplify launches LAYOUT_LAUNCHES expects run as their `ptrig` variant.
    calls: call lengths in place of the mode's of LAYOUT_MODES; env_extra: switches besides the entry's; size: (w, h, levels) in place of its"""
    idx, w, h, levels, env = LAYOUT_FORCED[force]
    w, h, levels = size or (w, h, levels)
    env = dict(env, **(env_extra or {}))
    if calls is None:
        worst, names = layout_case(lvm, po, lib, mem, idx, w, h, levels, n_streams, name, env=env, exact=exact, profile=True, clip_fn=clip_fn)
    else:
        _, over, clip_over = LAYOUT_MODES[idx]
        worst, names = layout_clip(lvm, po, lib, mem, idx, w, h, levels, n_streams, calls, LAYOUTS[name], env=env, over=over, clip_over=clip_over,
                                   exact=exact, profile=True, clip_fn=clip_fn)
    want = dict(LAYOUT_LAUNCHES[force]["*"], **LAYOUT_LAUNCHES[force][name])
    if ptrig:
        want = {n: ({"ptrig"} if n in PTRIG_NAMES and v == set() else v) for n, v in want.items()}
    for n, variants in want.items():
        if variants is None:
            assert n not in names, (force, name, n, names)
        else:
            assert n in names and names[n] == variants, (force, name, n, variants, names)
    return worst, {n: sorted(names[n]) for n, v in want.items() if v is not None}


# ---- many streams, full-length batches (tests/test_emu_many_streams.py, tests/test_gpu_exact.py, tests/test_gpu_riesz_exact.py) ---------
# In a batch the kernels see b = frame * n_streams + stream and take from it a stream's temporal state, a frame's planes and a wave's
# task.  bench.py runs 4 streams x 32 frames and 16 x 16 per call; the cases above stop at 3 streams and b of about 40.  Here: the
# benchmark's stream counts, 5 (odd: b / n and b % n are no shift and no mask) and 17 (one past 16), in calls of 16 and 32 frames (32 is
# Color's batch cap) and a short one behind them -- b reaches 32 * n_streams - 1: 511 at 16 streams, 543 at 17.  Every stream has a
# clip of its own (seed 1234 + stream), so output that lands in another stream's place, or state taken from it, changes bytes.
MANY_STREAMS = (4, 5, 16, 17)
MANY_TAIL = (16, 32, 3)
# per mode: the seeding calls (Laplace: the first frame; Riesz: the passthrough frame and the first filtered one; Color: 18 frames fill
# the window of COLOR_BATCH_PARAMS), parameter and clip overrides
MANY_MODES = {0: ((1,), None, None), 2: ((1, 1), None, None), 3: ((18,),) + COLOR_BATCH_PARAMS}
# (mode, w, h, levels): Laplace 64 x 48 takes the vector kernels and 67 x 45 the byte kernels
MANY_SHAPES = [(0, 64, 48, 3), (0, 67, 45, 2), (2, 64, 48, 2), (2, 67, 45, 2), (3, 40, 30, 1), (3, 64, 48, 2)]
MANY_CASES = [shape + (ns,) for shape in MANY_SHAPES for ns in MANY_STREAMS]
MANY_PER_FRAME = [(idx, ns) for idx in (0, 2, 3) for ns in (4, 16)]           # bench.py's per_frame_streams: lvm_process_device in a loop
MANY_PIPELINE = [(4, 4), (9, 4)]                                            # (frames, ring) of the 4-stream depth-1 pipeline
MANY_FORCED_STREAMS = 5
# With several streams the task count of "lap_rows" passes the threshold (it counts the CUs) from which lap_down0_lut replaces the pair
# lab_lut + lap_down0 that the entry is there for ("lap_fused" forces that kernel): the fused first kernel is switched off beside it.
MANY_FORCED_EXTRA = {"lap_rows": {"LVM_D0_FUSED": "0"}}
MANY_DEFAULT = (16, 16)                                                     # (streams, frames) of the default-flavour cases


def many_calls(idx, tail=MANY_TAIL):
    return MANY_MODES[idx][0] + tuple(tail)


def many_streams_case(lvm, po, lib, mem, idx, w, h, levels, ns, refs="libm", tail=MANY_TAIL, device=False, exact=True, profile_call=None):
    """One case of MANY_CASES through helpers.frames_clip, the oracle's frames from the shared cache (`refs`: "libm", or "ptrig" under
    portable_trig())."""
    seed, over, clip_over = MANY_MODES[idx]
    return frames_clip(lvm, po, lib, mem, idx, w, h, levels, ns, seed + tuple(tail), over, clip_over, refs=refs, device=device, exact=exact,
                       profile_call=profile_call)


def many_per_frame(lvm, po, lib, mem, idx, ns, refs="libm"):
    """six frames of every stream, one lvm_process_device call per frame (Color: behind the 18 frames that fill its window, per frame too)"""
    w, h, levels = [s[1:] for s in MANY_SHAPES if s[0] == idx][-1]
    return many_streams_case(lvm, po, lib, mem, idx, w, h, levels, ns, refs=refs, tail=(6,), device=True)


def many_forced(lvm, po, lib, mem, force, exact=True, ptrig=False, size=None):
    """an entry of LAYOUT_FORCED at MANY_FORCED_STREAMS streams on the view that keeps every strip kernel (B), the mode's seeding calls and a
    call of 9 frames: the bytes, and the kernels LAYOUT_LAUNCHES names.  size: a smaller (w, h, levels) for the emulation build"""
    idx = LAYOUT_FORCED[force][0]
    return layout_forced_case(lvm, po, lib, mem, force, "B", exact=exact, ptrig=ptrig, n_streams=MANY_FORCED_STREAMS, calls=many_calls(idx, (9,)),
                              env_extra=MANY_FORCED_EXTRA.get(force), size=size)


# ---- surfaces that lie far apart (helpers.far_clip): stream and frame strides of 2^31 + 64 and 2^32 + 128 bytes ------------------------------
# key -> (mode, w, h, levels, forced entry of LAYOUT_FORCED or None, odd base).  The default switches on the smallest shapes with w % 4 == 0
# (the far view is dword-aligned: vector kernels), Laplace once more from an odd base (byte kernels), and each mode's strip set of
# LAYOUT_FORCED at its own size, whose kernels build buffer resources on the far base: LAYOUT_LAUNCHES[...]["B"] must have run.
FAR_CASES = {
    "laplace": (0, 64, 48, 3, None, False), "laplace-odd-base": (0, 64, 48, 3, None, True), "laplace-rows": (0,) + LAYOUT_FORCED["lap_rows"][1:4] + ("lap_rows", False),
    "laplace-fused": (0,) + LAYOUT_FORCED["lap_fused"][1:4] + ("lap_fused", False),
    "riesz": (2, 64, 48, 2, None, False), "riesz-strips": (2,) + LAYOUT_FORCED["rz_strips"][1:4] + ("rz_strips", False),
    "color": (3, 64, 48, 2, None, False), "color-down01": (3,) + LAYOUT_FORCED["col_down01"][1:4] + ("col_down01", False),
    "color-out-rows": (3,) + LAYOUT_FORCED["col_out_rows"][1:4] + ("col_out_rows", False),
}


def far_case(lvm, po, lib, mem, key, refs="libm", ptrig=False):
    idx, w, h, levels, force, odd = FAR_CASES[key]
    seed, over, clip_over = MANY_MODES[idx]
    env = dict(LAYOUT_FORCED[force][4], **MANY_FORCED_EXTRA.get(force, {})) if force else None
    names = far_clip(lvm, po, lib, mem, idx, w, h, levels, sum(seed), over=over, clip_over=clip_over, env=env, odd=odd, refs=refs)
    if not force:
        return {n: sorted(v) for n, v in names.items()}
    want = dict(LAYOUT_LAUNCHES[force]["*"], **LAYOUT_LAUNCHES[force]["B"])
    if ptrig:
        want = {n: ({"ptrig"} if n in PTRIG_NAMES and v == set() else v) for n, v in want.items()}
    for n, variants in want.items():
        if variants is None:
            assert n not in names, (key, n, names)
        else:
            assert n in names and names[n] == variants, (key, n, variants, names)
    return {n: sorted(names[n]) for n, v in want.items() if v is not None}


# The other device surfaces that take a stream or frame stride (helpers.far_units): two units 2^32 + 128 bytes apart against the bytes the
# surface gives on packed buffers, and where the oracle restates the surface, against the oracle.
def _far_noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(2,) + shape, dtype=np.uint8)


def far_preprocess(lvm, po, lib, mem):
    """lvm_preprocess_device, two streams: ROI + fractional INTER_AREA cells + the gray stage (67 x 45, divisor 4: tests/test_preprocess.py)"""
    w, h, ds, roi = 67, 45, 4, (0.1, 0.2, 0.7, 0.55)
    kw = dict(downscale=ds, roiEnabled=True, roiX=roi[0], roiY=roi[1], roiW=roi[2], roiH=roi[3])
    cpre, opre = lvm.to_c_preprocess(lvm.PreprocessParams(**kw), True), po.make_pre_params(grayscale=True, **kw)
    frames = _far_noise((h, w, 3), 41)
    ow, oh, och = po.preprocess_geometry(opre, w, h, 3)[4:]
    assert och == 1
    _, want = far_units(lvm, lib, mem, 2, [frames], ow * oh, lambda ctx, ins, out: ctx.preprocess_device(
        cpre, ins[0][0], w, h, 3, w * 3, ins[0][1], out[0], ow, out[1], mem.stream()))
    for s in range(2):
        assert np.array_equal(want[s].reshape(oh, ow), po.preprocess(frames[s], opre)), s


def far_compose(lvm, po, lib, mem):
    """lvm_compose_device, two streams, LeftRight"""
    w, h, LR = 64, 48, 1
    orig, proc = _far_noise((h, w, 3), 42), _far_noise((h, w, 3), 43)
    ref = [po.compose(LR, orig[s], proc[s]) for s in range(2)]
    chh, cw = ref[0].shape[:2]
    _, want = far_units(lvm, lib, mem, 2, [orig, proc], cw * chh * 3, lambda ctx, ins, out: ctx.compose_device(
        LR, ins[0][0], w, h, 3, w * 3, ins[0][1], ins[1][0], w, h, 3, w * 3, ins[1][1], out[0], cw * 3, out[1], mem.stream()))
    for s in range(2):
        assert np.array_equal(want[s].reshape(ref[s].shape), ref[s]), s


def far_overlay(lvm, po, lib, mem):
    """lvm_overlay_device, two frames, in place (the tables of tests/test_export.py)"""
    cw, chh = 200, 40
    canvases = _far_noise((chh, cw, 3), 44)
    labels = [po.standin_label_tables(70, 14, 3, 6, 6, cw, chh, seed=4), po.standin_label_tables(80, 14, 3, 106, 6, cw, chh, seed=5)]
    _, want = far_units(lvm, lib, mem, 1, [], cw * chh * 3, lambda ctx, ins, out: ctx.overlay_device(out[0], cw, chh, 2, cw * 3, out[1], mem.stream()),
                        out_init=canvases, setup=lambda ctx: ctx.export_set_overlay(labels))
    for k in range(2):
        assert np.array_equal(want[k].reshape(chh, cw, 3), po.apply_overlay(canvases[k].copy(), labels)), k


def far_canvas_convert(lvm, po, lib, mem):
    """lvm_canvas_convert_device, two frames, NV12"""
    w, h = 64, 48
    frames = _far_noise((h, w, 3), 45)
    nbytes = w * h * 3 // 2

    def layout(ctx):
        assert ctx.canvas_layout(lvm.PIX_NV12, w, h, w)[0] == nbytes
    far_units(lvm, lib, mem, 1, [frames], nbytes, lambda ctx, ins, out: ctx.canvas_convert_device(
        lvm.PIX_NV12, ins[0][0], w, h, w * 3, ins[0][1], 2, out[0], w, out[1], mem.stream()), setup=layout)


def far_mjpeg_encode(lvm, po, lib, mem):
    """lvm_mjpeg_encode_device, two frames with a far frame_stride: the same JPEG bytes as from packed frames"""
    w, h = 64, 48
    ck, _ = lvm.synth.config(0, (w, h, 3))
    clip = lvm.synth.Clip(**ck)
    frames = np.stack([clip.frame(t) for t in range(2)])
    jpegs, _ = far_units(lvm, lib, mem, 1, [frames], 0, lambda ctx, ins, out: ctx.mjpeg_encode_device(ins[0][0], w, h, 2, stride=w * 3, frame_stride=ins[0][1]))
    assert len(jpegs) == 2 and jpegs[0] != jpegs[1] and all(j[:2] == b"\xff\xd8" and j[-2:] == b"\xff\xd9" for j in jpegs)


FAR_SURFACES = {"preprocess": far_preprocess, "compose": far_compose, "overlay": far_overlay, "canvas_convert": far_canvas_convert,
                "mjpeg_encode": far_mjpeg_encode}


class PatchedClip:
    """The synthetic clip with a flat black block, a flat white block and (from frame `const_from`) a constant frame:
    0/0 in the Riesz phase and amplitude steps (NaN patches, RieszPyramid.cpp:105-106,141), max == min in the colour
    normalisations (TemporalFilter.cpp:55, MagnifyCore.hpp:200-203)."""

    def __init__(self, clip, const_from=None):
        self.clip, self.const_from = clip, const_from

    def frame(self, t):
        f = self.clip.frame(t).copy()
        h, w = f.shape[:2]
        f[h // 8:h // 2, w // 8:w // 3] = 0
        f[h // 2:h - h // 8, w // 2:w - w // 8] = 255
        if self.const_from is not None and t >= self.const_from:
            f[...] = 77
        return f


FLAT_REGIONS = [(0, None, (96, 64, 3)), (2, None, (96, 64, 3)), (3, None, (96, 64, 3)), (0, 5, (96, 64, 3)), (2, 5, (96, 64, 3)),
                (3, 5, (96, 64, 3)),
                (2, None, (200, 120, 3))]   # black block wider than the 9x9 + 13x13 supports: exact 0/0


def flat_regions(lvm, po, lib, idx, const_from, size):
    ck, pk = lvm.synth.config(idx, size)
    if idx == 3:
        _color_fps(ck, pk)
    return run_pair(lvm, po, lib, PatchedClip(lvm.synth.Clip(**ck), const_from), pk, 9, 0.0, exact=True)


class ConstClip:
    def __init__(self, h, w, v):
        self.f = np.full((h, w, 3), v, np.uint8)

    def frame(self, t):
        return self.f


def fully_constant_clip(lvm, po, lib, idx):
    """Every frame the same constant: Color's output range collapses (max == min, 255 / 0 in convertTo:
    MagnifyCore.hpp:200-203), Riesz sees 0/0 in every phase difference, Laplace must return the Lab round trip."""
    ck, pk = lvm.synth.config(idx, (96, 64, 3))
    if idx == 3:
        pk["framerate"] = 15.0
    return run_pair(lvm, po, lib, ConstClip(64, 96, 131), pk, 8, 0.0, exact=True)


EXTREME_PARAMETERS = [(3, dict(coLow=5.0, coHigh=1.0)),                # colour: empty pass band (mask all zero)
                      (3, dict(coLow=0.0, coHigh=0.3)),                # colour: lo == 0 -> 0.01, DC excluded, first bins
                      (2, dict(coLow=0.5, coHigh=20.0)),               # Riesz: cutoff above Nyquist (Wn > 1)
                      (2, dict(coLow=0.5, coHigh=15.0)),               # Riesz: cutoff exactly at Nyquist (Wn == 1)
                      (2, dict(coLow=3.0, coHigh=1.0)),                # Riesz: hi < lo
                      (0, dict(amplification=1000.0, chromAttenuation=1.0)),   # Laplace: far out of gamut
                      (0, dict(amplification=0.0)),
                      (2, dict(amplification=0.0, coWavelength=0.0))]  # Riesz: zero gain / zero threshold


def extreme_parameters(lvm, po, lib, idx, over, kind=None):
    ck, pk = lvm.synth.config(idx, (96, 64, 3))
    if idx == 3:
        _color_fps(ck, pk)
    pk.update(over)
    return run_pair(lvm, po, lib, _clip(lvm, ck, kind), pk, 8, 0.0, exact=True)


class ShapeShifter:
    """Frames whose size / channel count changes mid-stream (the structural tracker must drop all state:
    MagnifyCore.hpp:53-65) and changes back."""

    def __init__(self, lvm, ck):
        self.a = lvm.synth.Clip(**ck)
        k2 = dict(ck); k2["w"], k2["h"] = 80, 48
        self.b = lvm.synth.Clip(**k2)

    def frame(self, t):
        if t < 4:
            return self.a.frame(t)
        if t < 7:
            return self.b.frame(t)                       # smaller frame
        if t < 10:
            return np.ascontiguousarray(self.a.frame(t)[:, :, 1])   # gray frame of the first size
        return self.a.frame(t)


def size_and_channel_changes(lvm, po, lib, idx):
    ck, pk = lvm.synth.config(idx, (96, 64, 2))
    if idx == 3:
        _color_fps(ck, pk)
    return run_pair(lvm, po, lib, ShapeShifter(lvm, ck), pk, 13, 0.0, exact=True)


def no_riesz(cases):
    """the entries of a matrix list whose first element (synth.config index) is not Riesz"""
    return [c for c in cases if c[0] != 2]


# ---- chromatic content (tests/content.py) ---------------------------------------------------------------------------------------
# Every case above draws its pixels from synth.texture, a grey grating: B, G and R of a pixel stay within about 30 levels of each
# other, which reads 5 % of the forward Lab table (tests/test_lab_lut.py: test_chromatic_content_reaches_the_table_off_the_grey_diagonal)
# and one branch combination of the inverse conversion.  The cases below send saturated colours through the same kernels: the cell
# and weight fields of the table index, its neighbours and padding plane, the mixed cubic / linear branches of Lab -> BGR, channels
# clamped at 0 beside channels clamped at 1.
# (mode, w, h, levels): the odd width takes the byte kernels; Color at 15 fps for 14 frames (the window fills, as in COLOR_SHAPES)
CHROMA_SHAPES = [(0, 96, 64, 3), (0, 67, 45, 2), (2, 96, 64, 3), (2, 67, 45, 2), (3, 64, 48, 2)]
CHROMA_CASES = [(kind, idx, w, h, levels) for kind in content.KINDS for (idx, w, h, levels) in CHROMA_SHAPES]
CHROMA_FORCED_KINDS = ("noise", "bars")


def chroma_shape(lvm, po, lib, kind, idx, w, h, levels, flavour_exact=True, bit_exact=None, channels=3):
    """One kind of content through one mode.  flavour_exact: OpenCV-order Lab (lvm_debug_exact_lab), else the default flavour;
    bit_exact (default: flavour_exact): float frames and bytes equal to the oracle's, else the project's bars (1e-4 relative, 1 LSB,
    >= 0.999 identical bytes) -- Riesz on the GPU in either flavour (device acosf / sinf / cosf)."""
    bit_exact = flavour_exact if bit_exact is None else bit_exact
    assert flavour_exact or not bit_exact
    ck, pk = lvm.synth.config(idx, (w, h, levels))
    ck["channels"] = channels
    if idx == 3:
        _color_fps(ck, pk)
    return run_pair(lvm, po, lib, content.chroma_clip(lvm, ck, kind), pk, 14 if idx == 3 else 6, 0.0 if bit_exact else 1e-4,
                    exact=bit_exact, exact_lab=flavour_exact)


def chroma_gray(lvm, po, lib):
    """Laplace on one-channel frames of `noise` (the clip's channel pick): no Lab on the way, grey-exact"""
    return chroma_shape(lvm, po, lib, "noise", 0, 96, 64, 3, channels=1)


CHROMA_FORCED_CASES = [(kind, force) for kind in CHROMA_FORCED_KINDS for force in LAYOUT_FORCED]


def chroma_forced(lvm, po, lib, mem, kind, force, exact=True, ptrig=False):
    """an entry of LAYOUT_FORCED at its own size and switches on the view that keeps every strip kernel (B): the bytes, and the
    kernels LAYOUT_LAUNCHES names"""
    return layout_forced_case(lvm, po, lib, mem, force, "B", exact=exact, clip_fn=content.clip_fn(lvm, kind), ptrig=ptrig)


CHROMA_ANALYTIC = [(kind,) + a for kind in CHROMA_FORCED_KINDS for a in (ANALYTIC[0], ANALYTIC[2])]

# temporal batches of `noise`: (mode, w, h, levels, streams, calls, parameter overrides, clip overrides)
CHROMA_BATCHES = [(0, 160, 90, 3, 2, (1, 4, 3), None, None), (2, 96, 64, 3, 1, (2, 5, 3), None, None),
                  (3, 64, 48, 2, 1, (18, 5, 7)) + COLOR_BATCH_PARAMS]
PACKED = (0, 0, 0, 0, 0, 0, "fs")          # helpers.layout_clip's geometry of packed rows, [frame][stream]


def chroma_batches(lvm, po, lib, mem, idx, w, h, levels, ns, calls, over, clip_over, exact=True):
    """exact=False (Riesz on the GPU): the bars of helpers.layout_clip on packed frames"""
    fn = content.clip_fn(lvm, "noise")
    if exact:
        return frames_clip(lvm, po, lib, mem, idx, w, h, levels, ns, calls, over, clip_over, clip_fn=fn)
    return layout_clip(lvm, po, lib, mem, idx, w, h, levels, ns, calls, PACKED, over=over, clip_over=clip_over, exact=False, clip_fn=fn)[0]


CHROMA_LAYOUTS = [(idx,) + LAYOUT_SHAPES[idx][0] + (name,) for idx in (0, 2) for name in ("A", "B", "D")]


def chroma_layout(lvm, po, lib, mem, idx, w, h, levels, name, exact=True):
    return layout_case(lvm, po, lib, mem, idx, w, h, levels, 1, name, exact=exact, clip_fn=content.clip_fn(lvm, "noise"))


def chroma_out_of_gamut(lvm, po, lib):
    """saturated hues amplified a thousandfold at full chroma: Lab far outside the gamut on every side of it"""
    assert EXTREME_PARAMETERS[5] == (0, dict(amplification=1000.0, chromAttenuation=1.0))
    return extreme_parameters(lvm, po, lib, *EXTREME_PARAMETERS[5], kind="hue")


# ---- launch switches and run-time instantiations (tests/test_emu_switches.py, tests/test_gpu_switches.py) ----------------------------
# Every LVM_* switch the launch code reads and no other test sets, and every kernel instantiation the launch code picks from a frame
# or level count.  A case is (mode, (w, h, levels), streams, call lengths, switches, check): the clip goes through
# lvm_process_device_frames in those calls, OpenCV-order Lab, with profiling on; the bytes of every frame and the float frame of every
# call's first frame (1-stream cases; Color: of 1-frame calls) must be the oracle's bit for bit -- Riesz on the GPU: the default kernels' on the same GPU -- and
# `check` gets, per call, {report name: variants} (lvm_profile_variants) and asserts the kernel the case is there for: a case that
# silently ran the default kernels fails.
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "live-video-magnification_amd", "csrc")


def up_tile():
    """(UT_W, UT_H): the tile of the LDS-tiled k_lap_up, read from csrc/pyramid.h"""
    text = open(os.path.join(_CSRC, "pyramid.h"), encoding="utf-8").read()
    return tuple(int(re.search(r"#define LVM_UT_%s (\d+)" % k, text).group(1)) for k in "WH")


def tiled_up_blocks(w, h, ns):
    """workgroups of the tiled k_lap_up at level 1 of w x h BGR frames of ns streams (laplace.hip, lap_stage_a: grid.z = planes)"""
    tw, th = up_tile()
    w1, h1 = (w + 1) // 2, (h + 1) // 2
    return -(-w1 // tw) * -(-h1 // th) * 3 * ns


def _pow2_dividing(nt, cap):
    d = cap
    while d > 1 and nt % d:
        d //= 2
    return d


def _present(name, variants=None, calls=None):
    """`name` launched in every call (of `calls`: indices; default: all but the seeding first call), with exactly these variants"""
    def check(prof, nts):
        for k in (range(1, len(prof)) if calls is None else calls):
            assert name in prof[k], (name, k, nts[k], sorted(prof[k]))
            if variants is not None:
                assert prof[k][name] == set(variants), (name, k, nts[k], prof[k][name], variants)
    return check


def _absent(*names, calls=None):
    def check(prof, nts):
        for k in (range(len(prof)) if calls is None else calls):
            for name in names:
                assert not any(re.fullmatch(name, n) for n in prof[k]), (name, k, nts[k], sorted(prof[k]))
    return check


def _by_frames(name, fn):
    """per call after the first: `name` ran as exactly the variant fn(frames of the call)"""
    def check(prof, nts):
        for k in range(1, len(prof)):
            assert prof[k].get(name) == {fn(nts[k])}, (name, k, nts[k], prof[k].get(name), fn(nts[k]))
    return check


def _all(*checks):
    def check(prof, nts):
        for c in checks:
            c(prof, nts)
    return check


UP_CALLS = (1, 8, 4, 6, 3)         # every ring depth on a frame count it divides and on one it does not
_FIN = {"LVM_FIN_ROWS": "8", "LVM_FIN_MIN_TASKS": "0"}
_FPS7 = ({"framerate": 7.0}, {"fps": 7.0})            # Color: a window of 16 columns
_FPS15 = ({"framerate": 15.0}, {"fps": 15.0})
# level 1 of 132 x 1346 (66 x 673: two tile columns, the right one 2 pixels wide; 43 tile rows, the last one 1 pixel high) on four streams:
# 2 x 43 tiles x 12 planes = 1032 tiled workgroups, of the frames that reach the 1024 from which the launch code reads LVM_UP_DEPTH_BIG
# about the fewest pixels (tests assert the count from UT_W / UT_H: tiled_up_blocks)
BIG_UP = (132, 1346, 3, 4)

SWITCH_CASES = {}


def _case(key, idx, size, calls, env, check, ns=1, over=None, clip_over=None):
    assert key not in SWITCH_CASES, key
    SWITCH_CASES[key] = dict(idx=idx, size=size, ns=ns, calls=tuple(calls), env=env, check=check, over=over, clip_over=clip_over)


# odd intermediate sizes, a coarsest tile that is no multiple of 8, several tiles.  Per-frame calls, then one call of two frames: at the two
# small sizes the LDS-resident tail kernel builds the coarse levels of a per-frame call itself and leaves pyrDown fewer than three levels,
# so k_pyr_down_multi<3> runs there in the batch only (a batch has no tail kernel); at 1001 x 763 in every call.  (At 135 x 77 the tail kernel
# starts at level 1: a per-frame call has no pyrDown launch at all.)
for _s, _pf, _pf1 in [((330, 200, 6), (), (0, 1, 2)), ((135, 77, 4), (), ()), ((1001, 763, 5), (0, 1, 2), (0, 1, 2))]:
    _case("fuse_down3-%dx%d" % _s[:2], 0, _s, (1, 1, 1, 2), {"LVM_FUSE_DOWN": "3"}, _present("pyr_down3_l1", calls=_pf + (3,)))
    _case("fuse_down1-%dx%d" % _s[:2], 0, _s, (1, 1, 1, 2), {"LVM_FUSE_DOWN": "1"},
          _all(_present("pyr_down_l1", calls=_pf1 + (3,)), _absent(r"pyr_down[23]_l\d+")))
for _d in (1, 2, 4, 8):
    _case("up_depth%d" % _d, 0, (328, 109, 3), UP_CALLS, {"LVM_UP_ROWS": "0", "LVM_UP_DEPTH": str(_d)},
          _all(_by_frames("lap_up_l1", lambda nt, d=_d: "tiled d%d curn" % _pow2_dividing(nt, d)),
               _by_frames("lap_iir", lambda nt: "d%d" % _pow2_dividing(nt, 8))))
for _d in (2, 4, 8):
    _case("up_depth_big%d" % _d, 0, BIG_UP[:3], (1, 8, 4), {"LVM_UP_DEPTH_BIG": str(_d)},
          _by_frames("lap_up_l1", lambda nt, d=_d: "tiled d%d curn" % _pow2_dividing(nt, d)), ns=BIG_UP[3])
_case("up_rows_max_blocks", 0, BIG_UP[:3], (1, 8, 4), {"LVM_UP_ROWS_MAX_BLOCKS": "1000000"},
      _by_frames("lap_up_l1", lambda nt: "rows d4 curn"), ns=BIG_UP[3])
for _r in (1, 3, 4, 16):          # 16 is halved to <= 4 at these sizes, 3 to 3: the halving loop from a start that is no power of two
    for _s in ROWS_PYRDOWN:
        _case("pd_rows%d-%dx%d" % ((_r,) + _s[:2]), 0, _s, (1, 1, 1), {"LVM_ROWS_MIN_ELEMS": "0", "LVM_PD_ROWS": str(_r)},
              _present("pyr_down_rows_l1", calls=(0, 1, 2)))
_case("d0_rows0-laplace", 0, (328, 109, 3), (1, 1, 1), {"LVM_D0_ROWS": "0", "LVM_D0_MIN_TASKS": "0"}, _present("lap_down0", {"vec4"}, calls=(0, 1, 2)))
_case("d0_rows0-color", 3, (264, 90, 3), (7, 5, 1), {"LVM_D0_ROWS": "0", "LVM_D0_MIN_TASKS": "0", "LVM_COL_DOWN01": "0"},
      _all(_present("col_down0", {"vec4"}, calls=(0, 1)), _absent("col_down01")), over=_FPS15[0], clip_over=_FPS15[1])
for _r in (5, 16):                # a height below the launch code's own choices (6 .. 48) and one of them
    for _s in [t[:3] for t in FUSED_TABLE if t[3]]:
        _case("d0_fused_rows%d-%dx%d" % ((_r,) + _s[:2]), 0, _s, (1, 1, 1), {"LVM_D0_FUSED_WAVES": "1", "LVM_D0_FUSED_ROWS": str(_r)},
              _all(_present("lap_down0_lut", calls=(0, 1, 2)), _absent("lap_down0", "lab_lut")))
# persistent kernels: one workgroup (or a few) walks every strip of every frame -- the state carried from task to task
for _g in (1, 3):
    _case("d0_fused_groups%d" % _g, 0, (328, 109, 3), (1, 4, 3), dict(_FIN, LVM_D0_FUSED_WAVES="1", LVM_D0_FUSED_GROUPS=str(_g)),
          _all(_present("lap_down0_lut", calls=(0, 1, 2)), _present("lap_final", {"strips"}, calls=(0, 1, 2))))
for _g in (1, 7):
    _case("fin_groups%d" % _g, 0, (328, 109, 3), (1, 4, 3), dict(_FIN, LVM_FIN_GROUPS=str(_g)), _present("lap_final", {"strips"}, calls=(0, 1, 2)))
for _g in (1, 5):                 # (the tiled last kernel is the persistent one: the strip form of level 0 switched off)
    _case("rz_fin_groups%d" % _g, 2, (264, 150, 3), (1, 4, 3), {"LVM_RZ_FIN_GROUPS": str(_g), "LVM_RZ_COLLAPSE_STRIPS": "0"},
          _present("rz_final", {"vec4"}))
_case("rz_phase4_0", 2, (264, 150, 3), (1, 4, 3), {"LVM_RZ_PHASE4": "0"}, _all(_present("rz_phase_small"), _absent("rz_phase")))
_RZ_TILES = {"LVM_RZ_SPLIT_ROWS": "0", "LVM_RZ_SPLIT2_MIN": "0"}          # the 9 x 9 split as tiles: 4 x 2 outputs per thread, or (LVM_RZ_SPLIT2=0) one
_case("rz_split2_default", 2, (264, 150, 3), (1, 4, 3), _RZ_TILES, _present("rz_split_l0", {"4x2"}, calls=(0, 1, 2)))
_case("rz_split2_0", 2, (264, 150, 3), (1, 4, 3), dict(_RZ_TILES, LVM_RZ_SPLIT2="0"), _present("rz_split_l0", {"tile"}, calls=(0, 1, 2)))
_SPLIT_CALLS = (1, 4, 1, 5, 2, 8)
_case("lap_split_min_nt4", 0, (320, 182, 5), _SPLIT_CALLS, {"LVM_LAP_SPLIT_MIN_NT": "4"},
      _all(_present("lap_iir", calls=[k for k, n in enumerate(_SPLIT_CALLS) if n >= 4]), _present("lap_collapse", calls=[k for k, n in enumerate(_SPLIT_CALLS) if n >= 4]),
           _absent("lap_iir", "lap_collapse", calls=[k for k, n in enumerate(_SPLIT_CALLS) if n < 4])))
for _k, (_lo, _hi) in enumerate(NARROW_DFT_BANDS):
    _case("col_thin_dft0-band%d" % _k, 3, (64, 48, 2), (18, 5, 7, 9), {"LVM_COL_THIN_DFT": "0"}, _present("col_dft", {"wave"}, calls=(0, 1, 2, 3)),
          over=dict(_FPS7[0], coLow=_lo, coHigh=_hi), clip_over=_FPS7[1])
# the window (16 columns) is full after the first call: from then on 1- and 2-frame calls take the wave-per-row kernel, the others the thin one
_THIN_CALLS = (18, 1, 5, 2, 4, 1)
_case("col_thin_min_frames4", 3, (64, 48, 2), _THIN_CALLS, {"LVM_COL_THIN_MIN_FRAMES": "4"},
      _all(_present("col_dft", {"wave"}, calls=(1, 3, 5)), _present("col_dft", {"thin8-128"}, calls=(2, 4))),
      over=dict(_FPS7[0], coLow=0.8, coHigh=1.6), clip_over=_FPS7[1])
# The first pyrUp of the up chain is a k_pyr_up_rows launch where the top level's width is even, and then the default normalises inside it.
# 96 x 64 and 528 x 90 (top levels 12 and 66 wide) are such: the switches move them to the other path.  264 x 90 (top level 33 wide) takes
# the tiled pyrUp and k_col_norm whatever the switches say.
for _s, _even in [((96, 64, 3), True), ((264, 90, 3), False), ((528, 90, 3), True)]:
    _on = _all(_present("col_norm", calls=(0, 1, 2)), _present("pyr_up_l0", {"rows" if _even else "tiled"}, calls=(0, 1, 2)))
    _case("col_up_default-%dx%d" % _s[:2], 3, _s, (7, 5, 1), {},
          _all(_absent("col_norm"), _present("pyr_up_l0", {"rows-norm"}, calls=(0, 1, 2))) if _even else _on, over=_FPS15[0], clip_over=_FPS15[1])
    _case("col_norm_in_up0-%dx%d" % _s[:2], 3, _s, (7, 5, 1), {"LVM_COL_NORM_IN_UP": "0"}, _on, over=_FPS15[0], clip_over=_FPS15[1])
    _case("col_up_rows0-%dx%d" % _s[:2], 3, _s, (7, 5, 1), {"LVM_COL_UP_ROWS": "0"},
          _all(_present("col_norm", calls=(0, 1, 2)), _present("pyr_up_l0", {"tiled"}, calls=(0, 1, 2))), over=_FPS15[0], clip_over=_FPS15[1])
# k_lap_collapse<N>, N = levels - F: F = 3 in calls of >= 4 frames (from 5 levels on), else 2.  N = 7 needs 9 levels, N = 8 ten.
# N = 9 and N = 10 need frames of at least 5121 x 5121 and 10241 x 10241 (lvm_max_levels = 11, 12): compiled, not tested.
DEEP = {4: (320, 180), 6: (256, 256), 7: (512, 384), 8: (1024, 768), 9: (1536, 1284), 10: (3072, 2564)}


def _collapse_n(levels):
    return lambda nt: "n%d" % (levels - (3 if nt >= 4 and levels >= 5 else 2))


for _lv, _wh in DEEP.items():
    _case("deep%d" % _lv, 0, _wh + (_lv,), (1, 2) if _lv in (4, 10) else (1, 4, 2), {}, _by_frames("lap_collapse", _collapse_n(_lv)))
# the defaults and the two-level pyramid (level 1 is the top live level: no cur_2 to add) for the ledger of instantiations
_case("up_default", 0, (328, 109, 3), UP_CALLS, {}, _by_frames("lap_up_l1", lambda nt: "rows d%d curn" % _pow2_dividing(nt, 4)))
_case("up_default-2levels", 0, (320, 180, 2), UP_CALLS, {}, _by_frames("lap_up_l1", lambda nt: "rows d%d" % _pow2_dividing(nt, 4)))
_case("up_tiled-2levels", 0, (320, 180, 2), UP_CALLS, {"LVM_UP_ROWS": "0"}, _by_frames("lap_up_l1", lambda nt: "tiled d%d" % _pow2_dividing(nt, 8)))
_NARROW = dict(_FPS7[0], coLow=0.8, coHigh=1.6)
_case("col_dft_thin8", 3, (64, 48, 2), (18, 5, 1), {}, _present("col_dft", {"thin8-128"}, calls=(0, 1)), over=_NARROW, clip_over=_FPS7[1])
_case("col_dft_thin", 3, (64, 48, 2), (18, 5, 1), {"LVM_COL_THIN8_DFT": "0"}, _present("col_dft", {"thin"}, calls=(0, 1)), over=_NARROW, clip_over=_FPS7[1])
# 0.8-3.3 Hz at 7 fps: the full 16-frame window passes the bins 2 .. 7 and the Nyquist element, seven entries -- more than k_col_dft_thin8's
# four, so the thread-per-row kernel with no switch set, and its loops over five to eight entries (the shorter windows of the first call have
# fewer entries and take other kernels: the check is on the calls with the full window)
_case("col_dft_thin_7entries", 3, (64, 48, 2), (18, 5, 1), {}, _present("col_dft", {"thin"}, calls=(1, 2)), over=dict(_FPS7[0], coLow=0.8, coHigh=3.3),
      clip_over=_FPS7[1])
_case("col_dft_long", 3, (64, 48, 2), (18, 5, 1), {"LVM_COL_LONG_FROM": "2"}, _present("col_dft", {"long"}, calls=(0, 1)), over=_NARROW, clip_over=_FPS7[1])
_case("col_dft_serial", 3, (64, 48, 2), (18, 5, 1), {"LVM_COL_LONG_FROM": "2", "LVM_COL_LONG_DFT": "0"}, _present("col_dft", {"serial"}, calls=(0, 1)),
      over=_NARROW, clip_over=_FPS7[1])
# a window of 129 .. 256 columns (120 fps: 256): k_col_dft_thin8<kThin8MaxN> once 129 frames are in
_case("col_dft_thin8_256", 3, (40, 30, 1), (120, 12, 8), {}, _all(_present("col_dft", {"thin8-128"}, calls=(0,)), _present("col_dft", {"thin8"}, calls=(2,))),
      over={"framerate": 120.0, "coLow": 0.8, "coHigh": 1.6}, clip_over={"fps": 120.0})

# What the launch code can pick at run time, as (report name without its level, variant): the ledger tests assert that the cases above reach
# every one.  k_lap_collapse<9> and <10> are left out (unreachable below 5121 x 5121 and 10241 x 10241, see DEEP).
REQUIRED = ({("lap_up", "%s d%d%s" % (k, d, c)) for k, ds in (("rows", (1, 2, 4)), ("tiled", (1, 2, 4, 8))) for d in ds for c in ("", " curn")}
            | {("lap_iir", "d%d" % d) for d in (1, 2, 4, 8)} | {("lap_collapse", "n%d" % n) for n in range(2, 9)}
            | {("col_dft", v) for v in ("thin8-128", "thin8", "thin", "wave", "long", "serial")})


# Values the validators of the switches refuse (csrc: laplace_switches): the default must run.  Emulation only -- the point of the validators is
# that such a value never reaches a kernel, so these are kept apart from SWITCH_CASES and no GPU test runs them.
_ROWS_ON = {"LVM_ROWS_MIN_ELEMS": "0"}
REFUSED_CASES = {
    # a ring of 3 (6) would launch k_lap_up<false, 4> (<8>) on 3 (6) frames: a frame past the batch.  Refused: the default 8, halved to fit
    "refused-up_depth3": (0, (328, 109, 3), (1, 3, 3), {"LVM_UP_ROWS": "0", "LVM_UP_DEPTH": "3"}, _present("lap_up_l1", {"tiled d1 curn"})),
    "refused-up_depth6": (0, (328, 109, 3), (1, 6), {"LVM_UP_ROWS": "0", "LVM_UP_DEPTH": "6"}, _present("lap_up_l1", {"tiled d2 curn"})),
    "refused-pd_rows0": (0, (328, 109, 3), (1, 1, 1), dict(_ROWS_ON, LVM_PD_ROWS="0"), _present("pyr_down_rows_l1", calls=(0, 1, 2))),
    "refused-pd_rows-4": (0, (328, 109, 3), (1, 1, 1), dict(_ROWS_ON, LVM_PD_ROWS="-4"), _present("pyr_down_rows_l1", calls=(0, 1, 2))),
    "refused-fin_groups-1": (0, (328, 109, 3), (1, 4, 3), dict(_FIN, LVM_FIN_GROUPS="-1"), _present("lap_final", {"strips"}, calls=(0, 1, 2))),
    # 7 would read as ">= 3", the three-level kernel.  Refused: the default, two levels per launch
    "refused-fuse_down7": (0, (330, 200, 6), (1, 1, 2), {"LVM_FUSE_DOWN": "7"},
                           _all(_present("pyr_down2_l1", calls=(2,)), _absent(r"pyr_down3_l\d+"))),
}
REFUSED_SWITCH = {"refused-up_depth3": "LVM_UP_DEPTH", "refused-up_depth6": "LVM_UP_DEPTH", "refused-pd_rows0": "LVM_PD_ROWS",
                  "refused-pd_rows-4": "LVM_PD_ROWS", "refused-fin_groups-1": "LVM_FIN_GROUPS", "refused-fuse_down7": "LVM_FUSE_DOWN"}


# ---- the portable functions (LVM_RZ_PORTABLE_TRIG + LVMO_VAR_PORTABLE_TRIG): one case per instantiation that calls them --------------
# k_rz_phase / k_rz_phase4 <true, UNF, MF32, true> under every build kind of (UNF, MF32), and the three forms of the blur / amplify stage --
# wave strips (with the out-of-line rz_amplify_ptrig_call), register-blocked tiles, scalar tiles -- <true, UNF, true>.  Run by
# tests/test_emu_portable_trig.py and tests/test_gpu_riesz_exact.py through switch_case under portable_trig(): bytes and float frames
# equal to the oracle's, and every phase and blur / amplify launch reported as the `ptrig` variant of its kind.  Sizes: 264 x 150 L3
# (levels 264 and 132 wide: four pixels per thread, register-blocked tiles) and 134 x 78 L2 (2 mod 4: the scalar kernels, strips).
PTRIG_CASES = {}
_CV_UNFUSED, _CV_MUL_F32 = 1, 4                               # LVM_CV_* (include/lvm_hip.h)
_KIND_BITS = {0: (), _CV_UNFUSED: ("filter_unfused",), _CV_MUL_F32: ("mul_f32",), _CV_UNFUSED | _CV_MUL_F32: ("filter_unfused", "mul_f32")}
_KIND_PHASE = {0: "ptrig", _CV_UNFUSED: "unfused+ptrig", _CV_MUL_F32: "mulf32+ptrig", _CV_UNFUSED | _CV_MUL_F32: "unfused+mulf32+ptrig"}


def _ptrig_check(want, absent=()):
    def check(prof, nts):
        for k in range(1, len(prof)):
            got = ptrig_launches(prof[k])
            assert got == {n: {v} for n, v in want.items()}, (k, nts[k], got, want)
            assert not any(n in prof[k] for n in absent), (k, absent, sorted(prof[k]))
    return check


def _ptrig_case(key, size, env, want, kind=0):
    assert key not in PTRIG_CASES and key not in SWITCH_CASES, key
    PTRIG_CASES[key] = dict(idx=2, size=size, ns=1, calls=(1, 1, 3, 2), env=env, check=_ptrig_check(want), over=None, clip_over=None, kind=kind,
                            oracle_bits=_KIND_BITS[kind])


for _kind in _KIND_BITS:
    _blur = "unfused+ptrig" if _kind & _CV_UNFUSED else "ptrig"
    _case_tail = "" if not _kind else "-" + _KIND_PHASE[_kind].replace("+ptrig", "")
    _ptrig_case("ptrig-phase" + _case_tail, (134, 78, 2), {}, {"rz_phase_small": _KIND_PHASE[_kind], "rz_blur_amp": _blur}, _kind)
    _ptrig_case("ptrig-phase4" + _case_tail, (264, 150, 3), {"LVM_RZ_PHASE4_MIN_FRAMES": "1"}, {"rz_phase": _KIND_PHASE[_kind], "rz_blur_amp": _blur}, _kind)
for _kind in (0, _CV_UNFUSED):
    _blur = "unfused+ptrig" if _kind else "ptrig"
    _case_tail = "-unfused" if _kind else ""
    _tiles = {"LVM_RZ_BLUR_STRIPS": "0", "LVM_RZ_PHASE4_MIN_FRAMES": "1"}
    _ptrig_case("ptrig-blur-blocked" + _case_tail, (264, 150, 3), dict(_tiles, LVM_RZ_BLUR4="1"), {"rz_phase": _KIND_PHASE[_kind], "rz_blur_amp": _blur}, _kind)
    _ptrig_case("ptrig-blur-tiled" + _case_tail, (264, 150, 3), dict(_tiles, LVM_RZ_BLUR4="0"), {"rz_phase": _KIND_PHASE[_kind], "rz_blur_amp_small": _blur}, _kind)
# the smallest shape of tests/test_gpu_opencv_build.py (odd sizes: byte I/O, the scalar tile kernels) under the two kinds the header meets
for _kind in (_CV_UNFUSED, _CV_MUL_F32):
    _ptrig_case("ptrig-67x131-" + _KIND_PHASE[_kind].replace("+ptrig", ""), (67, 131, 2), {},
                {"rz_phase_small": _KIND_PHASE[_kind], "rz_blur_amp_small": "unfused+ptrig" if _kind & _CV_UNFUSED else "ptrig"}, _kind)
_ptrig_case("ptrig-blur-strips16", (264, 150, 3), {"LVM_RZ_BLUR_STRIPS_MIN": "0", "LVM_RZ_BLUR_STRIP_ROWS": "16", "LVM_RZ_PHASE4_MIN_FRAMES": "1"},
            {"rz_phase": "ptrig", "rz_blur_amp": "ptrig"})


def _lookup(key):
    if key in SWITCH_CASES:
        return SWITCH_CASES[key]
    if key in PTRIG_CASES:
        return PTRIG_CASES[key]
    idx, size, calls, env, check = REFUSED_CASES[key]
    return dict(idx=idx, size=size, ns=1, calls=calls, env=env, check=check, over=None, clip_over=None)


def switch_run(lvm, lib, mem, key, env=None):
    """the library's side of SWITCH_CASES[key] (env: the switches, default the case's): per call (input frames, produced flags, output
    frames, float frame of the call's first frame or None, {report name: variants})"""
    c = _lookup(key)
    w, h, levels = c["size"]
    ns = c["ns"]
    ck, pk = lvm.synth.config(c["idx"], c["size"])
    pk.update(c["over"] or {})
    ck.update(c["clip_over"] or {})
    clips = [lvm.synth.Clip(seed=1234 + s, **ck) for s in range(ns)]
    env = c["env"] if env is None else env
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    ctx, res, t, fb = None, [], 0, w * h * 3
    try:
        ctx = lvm.Context(0, ns, lib)
        ctx.exact_lab(True)
        ctx.keep_float(ns == 1)
        if c.get("kind"):
            ctx.set_opencv_build(c["kind"])
        ctx.profile(True)
        cp = lvm.LvmParams(pk["mode"], pk["levels"], pk["amplification"], pk["coWavelength"], pk["coLow"], pk["coHigh"], pk["chromAttenuation"],
                           pk["framerate"], 0)
        for nf in c["calls"]:
            fin = np.stack([np.stack([cl.frame(t + f) for cl in clips]) for f in range(nf)])      # [frame][stream][h][w][3]
            d_in = mem.upload(fin)
            d_out = mem.zeros_like(d_in)
            prod = ctx.process_device_frames(cp, nf, mem.ptr(d_in), w, h, 3, w * 3, fb, fb * ns, mem.ptr(d_out), w * 3, fb, fb * ns, mem.stream())
            mem.sync(ctx)
            out = np.array(mem.download(d_out), copy=True)
            # (Laplace and Riesz keep the float frame of a call's first frame, Color of its last: read after 1-frame calls)
            fl = ctx.read_float((h, w, 3)).copy() if ns == 1 and prod[0] and (nf == 1 or c["idx"] != 3) else None
            variants = ctx.profile_variants()
            names = {n: variants.get(n, set()) for n in ctx.profile_collect()}
            ctx.profile_only(None)                     # clears the report: the next call's launches on their own
            res.append((fin, list(prod), out, fl, names))
            t += nf
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if ctx is not None:
            ctx.close()
    return pk, res


_LAUNCHED = {}          # (build, case) -> per call {report name: variants}, of the cases that have passed in this process


def switch_case(lvm, po, lib, mem, build, key, reference="oracle"):
    """One case of SWITCH_CASES on the library `lib` (`build`: "emu" / "gpu", the ledger's key): bytes and float frames against the
    oracle, or (reference="default": Riesz on the GPU, device acosf / sinf / cosf) against the same library without the case's switches;
    then the case's check of what was launched.  Returns the launches per call; a case that has passed is not run again."""
    if (build, key) in _LAUNCHED:
        return _LAUNCHED[(build, key)]
    c = _lookup(key)
    pk, res = switch_run(lvm, lib, mem, key)
    if reference == "default":
        _, base = switch_run(lvm, lib, mem, key, env={})
        for k, ((_, prod, out, fl, _n), (_, bprod, bout, bfl, _m)) in enumerate(zip(res, base)):
            assert prod == bprod, (key, k, prod, bprod)          # (a frame that was not produced leaves its zeros in both)
            assert np.array_equal(out, bout), "%s call %d: %d bytes differ from the default kernels" % (key, k, int((out != bout).sum()))
            assert (fl is None) == (bfl is None) and (fl is None or np.array_equal(fl, bfl)), "%s call %d: float frames differ from the default kernels" % (key, k)
        assert any(p for r in res for p in r[1]), key
    else:
        P = po.make_params(**pk)
        orcs = [po.Oracle() for _ in range(c["ns"])]
        try:
            t = 0
            for k, (fin, prod, out, fl, _n) in enumerate(res):
                for f in range(len(prod)):
                    for s in range(c["ns"]):
                        ref, pr = orcs[s].process(fin[f, s], P)
                        assert prod[f] == pr, (key, t + f, prod[f], pr)
                        if not pr:
                            continue
                        assert np.array_equal(ref, out[f, s]), "%s frame %d stream %d: %d bytes differ from the oracle" % (
                            key, t + f, s, int((ref != out[f, s]).sum()))
                        if fl is not None and f == 0:
                            fr = orcs[s].last_float()
                            assert np.array_equal(fr, fl), "%s frame %d: %d float values differ from the oracle" % (key, t + f, int((fr != fl).sum()))
                t += len(prod)
        finally:
            for o in orcs:
                o.close()
    prof = [r[4] for r in res]
    c["check"](prof, list(c["calls"]))
    _LAUNCHED[(build, key)] = prof
    return prof


# the cases that between them launch all of REQUIRED ("deep10" where the build runs it)
LEDGER_KEYS = (["up_depth%d" % d for d in (1, 2, 4, 8)] + ["up_default", "up_default-2levels", "up_tiled-2levels", "col_thin_dft0-band0"]
               + ["deep%d" % lv for lv in DEEP] + ["col_dft_thin8", "col_dft_thin", "col_dft_long", "col_dft_serial", "col_dft_thin8_256"])


def ledger(lvm, po, lib, mem, build, keys, reference=None):
    """(report name without its level, variant) of everything the cases `keys` launch on this build (cases that have not run yet run now)"""
    seen = set()
    for key in keys:
        ref = (reference or {}).get(key, "oracle")
        for call in switch_case(lvm, po, lib, mem, build, key, ref):
            for name, variants in call.items():
                seen |= {(re.sub(r"_l\d+$", "", name), v) for v in variants}
    return seen
