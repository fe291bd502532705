"""The Laplace and Color cases that must equal the CPU oracle BIT FOR BIT in the exact flavour (lvm_debug_exact_lab: OpenCV's
operation order, no transcendental function on the way) -- one matrix, run on the CPU emulation build by tests/test_emu_parity.py
and on the gfx950 build by tests/test_gpu_exact.py.  Each body takes the library behind the C ABI (`lib`) and, where it passes
device pointers, a memory adaptor (helpers.HostMem / helpers.TorchMem).  Lists hold Riesz entries where the emulation test of the
same name covers all three modes; the GPU module keeps the Laplace and Color ones (Riesz calls acosf / sinf / cosf, see
tests/test_gpu_exact.py)."""
import numpy as np

import content
from helpers import frames_clip, layout_clip, run_pair


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


# ---- every mode: layouts, degenerate content, parameters, shapes ----------------------------------------------------------
PADDED_STRIDES = [(0, 4, 8), (0, 1, 3), (2, 4, 4), (2, 7, 1), (3, 8, 4), (3, 5, 5)]


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


def layout_forced_case(lvm, po, lib, mem, force, name, exact=True, clip_fn=None):
    """one forced case: the bytes, and the kernels LAYOUT_LAUNCHES names for this layout -- a silent fall-back to another kernel family fails"""
    idx, w, h, levels, env = LAYOUT_FORCED[force]
    worst, names = layout_case(lvm, po, lib, mem, idx, w, h, levels, 1, name, env=env, exact=exact, profile=True, clip_fn=clip_fn)
    want = dict(LAYOUT_LAUNCHES[force]["*"], **LAYOUT_LAUNCHES[force][name])
    for n, variants in want.items():
        if variants is None:
            assert n not in names, (force, name, n, names)
        else:
            assert n in names and names[n] == variants, (force, name, n, variants, names)
    return worst, {n: sorted(names[n]) for n, v in want.items() if v is not None}


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


def chroma_forced(lvm, po, lib, mem, kind, force, exact=True):
    """an entry of LAYOUT_FORCED at its own size and switches on the view that keeps every strip kernel (B): the bytes, and the
    kernels LAYOUT_LAUNCHES names"""
    return layout_forced_case(lvm, po, lib, mem, force, "B", exact=exact, clip_fn=content.clip_fn(lvm, kind))


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
